// dhcp_table.cc — the DHCP server object: lease table and state machine (dhcp_table.h). Each
// handler restates its lines of engine/dhcp_engine.go call for call, quirks included.
#include "dhcp_table.h"

#include <string.h>

#include <new>

namespace {

constexpr uint32_t kLeaseTime = 3600;  // DhcpLeaseTime

halo_dhcp_reply_t reply_of(uint32_t kind, const uint8_t xid[4], uint32_t yiaddr, const uint8_t chaddr[6]) {
    halo_dhcp_reply_t r;
    memset(&r, 0, sizeof r);
    r.kind = (uint8_t)kind, r.yiaddr = yiaddr;
    memcpy(r.xid, xid, 4);
    memcpy(r.chaddr, chaddr, 6);
    return r;
}

struct Out {
    halo_dhcp_reply_t* replies;
    uint32_t n_replies;
    halo_dhcp_client_event_t* events;
    uint32_t n_events;
};

// dhcp_engine.go:234-288
uint8_t on_discover(halo_dhcp_server* s, const halo_dhcp_msg_t& m, Out& out) {
    uint8_t flags = 0;
    uint32_t client = 0;
    if (m.options & HALO_DHCP_OPT_REQ_IP) {
        const auto it = s->leases.find(m.req_ip);
        if (it != s->leases.end() && !memcmp(it->second.mac, m.chaddr, 6)) client = m.req_ip, flags = HALO_DHCP_H_F_REUSED;
    }
    if (client == 0) {
        flags = 0;  // a lease for address 0 "reused" is no address: the scan runs, as in the reference
        const uint32_t self = s->cfg.ip, network = self & s->cfg.network_mask;
        const uint32_t host_bits = 32u - (uint32_t)__builtin_popcount(network);  // of the network ADDRESS, as written
        if (host_bits < 32u) {
            for (uint32_t ii = 0; ii < (1u << host_bits); ++ii) {
                const uint32_t ip = network + ii;
                if ((uint8_t)ip == 0 || (uint8_t)ip == 255 || ip == self || s->leases.count(ip)) continue;
                client = ip;
                break;
            }
        }
    }
    if (client == 0) return HALO_DHCP_H_NO_ADDR;
    out.replies[out.n_replies++] = reply_of(HALO_DHCP_OFFER, m.xid, client, m.chaddr);
    return HALO_DHCP_H_OFFER | flags | HALO_DHCP_H_F_REPLY;
}

// dhcp_engine.go:289-347
uint8_t on_request(halo_dhcp_server* s, const halo_dhcp_msg_t& m, uint64_t now, Out& out) {
    if (!(m.options & HALO_DHCP_OPT_REQ_IP)) return HALO_DHCP_H_NO_REQ_IP;
    uint8_t code = HALO_DHCP_H_ACK_NAK, flags = 0;
    const uint32_t req = m.req_ip, mask = s->cfg.network_mask;
    const auto it = s->leases.find(req);
    const bool exist = it != s->leases.end();
    if (req == 0) code = HALO_DHCP_H_NAK_ZERO;
    else if ((s->cfg.ip & mask) != (req & mask)) code = HALO_DHCP_H_NAK_SUBNET;
    else if (exist && memcmp(it->second.mac, m.chaddr, 6)) code = HALO_DHCP_H_NAK_OTHER_MAC;
    else if (!exist && s->leases.size() >= s->cfg.capacity) code = HALO_DHCP_H_NAK_FULL;
    if (code == HALO_DHCP_H_ACK_NAK) {
        const uint32_t hn = (m.options & HALO_DHCP_OPT_HOSTNAME) ? m.hostname[63] : 0u;
        if (hn == 0) return HALO_DHCP_H_REF_PANIC;  // StaticString64.Set(""): no state change, no reply
        halo_dhcp_lease_t fresh;
        memset(&fresh, 0, sizeof fresh);
        halo_dhcp_lease_t& l = exist ? it->second : fresh;
        l.ip = req;
        memcpy(l.mac, m.chaddr, 6);
        l.exp_time = (uint32_t)(now + kLeaseTime);
        l.hostname[63] = (uint8_t)hn;  // Set: the count, then MemCpy of that many bytes; the rest stays
        memcpy(l.hostname, m.hostname, hn);
        if (exist) flags = HALO_DHCP_H_F_REUSED;
        else s->leases.emplace(req, fresh);
        out.replies[out.n_replies++] = reply_of(HALO_DHCP_ACK, m.xid, req, m.chaddr);
        // no return in front of the dhcp_nak label: the NAK follows the ACK
    }
    out.replies[out.n_replies++] = reply_of(HALO_DHCP_NAK, m.xid, 0, m.chaddr);
    return code | flags | HALO_DHCP_H_F_REPLY;
}

// dhcp_engine.go:358-433
uint8_t on_client(halo_dhcp_server* s, const halo_dhcp_msg_t& m, uint32_t i, Out& out) {
    if (s->cfg.ip != 0) return HALO_DHCP_H_NONE;
    if (!s->client_xid_set || memcmp(m.xid, s->client_xid, 4)) return HALO_DHCP_H_NONE;
    if (!(m.options & HALO_DHCP_OPT_MSG_TYPE)) return HALO_DHCP_H_NONE;
    if (m.msg_type == HALO_DHCP_OFFER) {
        halo_dhcp_reply_t r = reply_of(HALO_DHCP_REQUEST, m.xid, 0, s->cfg.mac);
        r.req_ip = m.yiaddr, r.server_id = m.remote_ip;
        out.replies[out.n_replies++] = r;
        return HALO_DHCP_H_CLIENT_REQUEST | HALO_DHCP_H_F_REPLY;
    }
    if (m.msg_type == HALO_DHCP_ACK) {
        if (out.events) {
            halo_dhcp_client_event_t e;
            memset(&e, 0, sizeof e);
            e.msg = i, e.ip = m.yiaddr;
            memcpy(e.mask, m.mask, 4), memcpy(e.gateway, m.gateway, 4), memcpy(e.dns, m.dns, 4);
            e.mask_n = m.mask_n, e.gateway_n = m.gateway_n;
            e.options = (uint8_t)(m.options & (HALO_DHCP_OPT_MASK | HALO_DHCP_OPT_ROUTER | HALO_DHCP_OPT_DNS));
            out.events[out.n_events] = e;
        }
        ++out.n_events;
        return HALO_DHCP_H_CLIENT_ACK;
    }
    return HALO_DHCP_H_NONE;
}

uint8_t handle(halo_dhcp_server* s, const halo_dhcp_msg_t& m, uint32_t i, uint64_t now, Out& out) {
    if (m.status != HALO_DHCP_OK) return HALO_DHCP_H_NONE;
    if (m.dir == HALO_DHCP_TO_CLIENT) return s->cfg.client_enable ? on_client(s, m, i, out) : HALO_DHCP_H_NONE;
    if (m.dir != HALO_DHCP_TO_SERVER || !s->cfg.server_enable || !(m.options & HALO_DHCP_OPT_MSG_TYPE)) return HALO_DHCP_H_NONE;
    switch (m.msg_type) {
        case HALO_DHCP_DISCOVER: return on_discover(s, m, out);
        case HALO_DHCP_REQUEST: return on_request(s, m, now, out);
        case HALO_DHCP_RELEASE: return s->leases.erase(m.remote_ip) ? HALO_DHCP_H_RELEASED : HALO_DHCP_H_RELEASE_ABSENT;  // :348-355
        default: return HALO_DHCP_H_NONE;
    }
}

}  // namespace

extern "C" {

HALO_API int halo_dhcp_server_create(const halo_dhcp_config_t* cfg, halo_dhcp_server_t** out) {
    if (!cfg || !out) return HALO_E_INVAL;
    halo_dhcp_server* s = new (std::nothrow) halo_dhcp_server();
    if (!s) return HALO_E_NOMEM;
    s->cfg = *cfg;
    s->cfg.server_enable = cfg->server_enable != 0, s->cfg.client_enable = cfg->client_enable != 0;
    memset(s->client_xid, 0, 4);
    s->client_xid_set = false;
    *out = s;
    return HALO_OK;
}

HALO_API void halo_dhcp_server_destroy(halo_dhcp_server_t* s) { delete s; }

HALO_API int halo_dhcp_handle_msgs(halo_dhcp_server_t* s, const halo_dhcp_msg_t* msgs, uint32_t n, uint64_t now,
                                   halo_dhcp_reply_t* replies, uint32_t reply_cap, uint8_t* verdicts, uint32_t* n_replies,
                                   halo_dhcp_client_event_t* events, uint32_t event_cap, uint32_t* n_events) {
    if (!s || !n_replies || (n && (!msgs || !replies))) return HALO_E_INVAL;
    if ((uint64_t)reply_cap < 2ull * n) return HALO_E_INVAL;
    if (events ? event_cap < n : event_cap != 0) return HALO_E_INVAL;
    Out out{replies, 0, events, 0};
    for (uint32_t i = 0; i < n; ++i) {
        halo_dhcp_msg_t m;  // no alignment asked of the caller's array
        memcpy(&m, reinterpret_cast<const uint8_t*>(msgs) + sizeof m * (uint64_t)i, sizeof m);
        const uint8_t v = handle(s, m, i, now, out);
        if (verdicts) verdicts[i] = v;
    }
    *n_replies = out.n_replies;
    if (n_events) *n_events = out.n_events;
    return HALO_OK;
}

HALO_API uint32_t halo_dhcp_list(const halo_dhcp_server_t* s, halo_dhcp_lease_t* out, uint32_t cap) {
    if (!s) return 0;
    uint32_t k = 0;
    for (const auto& kv : s->leases) {
        if (out && k < cap) memcpy(reinterpret_cast<uint8_t*>(out) + sizeof(halo_dhcp_lease_t) * (uint64_t)k, &kv.second, sizeof kv.second);
        ++k;
    }
    return k;
}

HALO_API uint32_t halo_dhcp_clear(halo_dhcp_server_t* s, uint64_t now) {
    if (!s) return 0;
    uint32_t gone = 0;
    const uint32_t time_now = (uint32_t)now;  // Router.TimeNow is a uint32
    for (auto it = s->leases.begin(); it != s->leases.end();) {
        if (time_now > it->second.exp_time) it = s->leases.erase(it), ++gone;
        else ++it;
    }
    return gone;
}

HALO_API int halo_dhcp_set_dns(halo_dhcp_server_t* s, uint32_t dns) {
    if (!s) return HALO_E_INVAL;
    s->cfg.dns = dns;
    return HALO_OK;
}

HALO_API int halo_dhcp_set_client_xid(halo_dhcp_server_t* s, const uint8_t xid[4]) {
    if (!s || !xid) return HALO_E_INVAL;
    memcpy(s->client_xid, xid, 4);
    s->client_xid_set = true;
    return HALO_OK;
}

HALO_API int halo_dhcp_discover(halo_dhcp_server_t* s, const uint8_t xid[4], halo_dhcp_reply_t* reply) {
    if (!reply) return HALO_E_INVAL;
    const int rc = halo_dhcp_set_client_xid(s, xid);
    if (rc) return rc;
    *reply = reply_of(HALO_DHCP_DISCOVER, xid, 0, s->cfg.mac);  // dhcp_engine.go:463-467
    return HALO_OK;
}

HALO_API int halo_dhcp_server_config(const halo_dhcp_server_t* s, halo_dhcp_config_t* out) {
    if (!s || !out) return HALO_E_INVAL;
    *out = s->cfg;
    return HALO_OK;
}

}  // extern "C"
