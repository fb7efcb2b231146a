// rx_kcp_host.cc — KCP ingest's C entry points (include/halo_rx.h, "KCP ingest"): the argument
// checks of halo_kcp_ingest_device, answered before any device is looked for, and
// halo_kcp_ingest_host, the sequential loop with the same outputs. No HIP: the kernels live in
// rx_kcp.hip behind kcp::device_ops(), and this file compiles alone with g++ (tools/fuzz_kcp.cc
// drives it under ASan/UBSan). The host byte checks are kcp_check_host.h's, shared with KCP emit.
#include <string.h>

#include "kcp_check_host.h"
#include "rx_kcp.h"

namespace halo {
namespace kcp {
namespace {

// What both entry points ask
int check(const halo_kcp_config_t* cfg, const uint8_t* stream, const halo_deliver_summary_t* dsum,
          const halo_deliver_index_t* index, uint32_t index_cap, const halo_kcp_dgram_t* dgrams, const halo_kcp_seg_t* segs,
          const halo_kcp_summary_t* summary) {
    if (!cfg || !summary || !dsum) return HALO_E_INVAL;
    if (!mode_ok(cfg->byte_check_mode) || cfg->port > 0xFFFFu) return HALO_E_INVAL;
    if (index_cap && (!stream || !index)) return HALO_E_INVAL;
    if ((cfg->dgram_cap && !dgrams) || (cfg->seg_cap && !segs)) return HALO_E_INVAL;
    return HALO_OK;
}

struct HostBytes {  // a payload in host memory, any alignment
    const uint8_t* p;
    uint32_t u32(uint32_t pos) const { return load_u32(p + pos); }
};

}  // namespace
}  // namespace kcp
}  // namespace halo

using namespace halo;  // host_layout.h
using namespace halo::kcp;

extern "C" HALO_API uint64_t halo_kcp_ingest_workspace(uint32_t index_cap, uint32_t seg_cap) {
    return kcp::workspace_bytes(index_cap, seg_cap);
}

extern "C" HALO_API int halo_kcp_ingest_device(const halo_kcp_config_t* cfg, const uint8_t* d_stream,
                                               const halo_deliver_summary_t* d_deliver_summary,
                                               const halo_deliver_index_t* d_index, uint32_t index_cap,
                                               halo_kcp_dgram_t* d_dgrams, halo_kcp_seg_t* d_segs,
                                               halo_kcp_summary_t* d_summary, void* d_workspace, uint64_t workspace_bytes,
                                               halo_stream_t stream) {
    int rc;
    if ((rc = check(cfg, d_stream, d_deliver_summary, d_index, index_cap, d_dgrams, d_segs, d_summary))) return rc;
    if (misaligned(d_segs, 16) || misaligned(d_dgrams, 8) || misaligned(d_index, 8) || misaligned(d_summary, 8) ||
        misaligned(d_deliver_summary, 8) || misaligned(d_workspace, 8) || misaligned(d_stream, 4))
        return HALO_E_INVAL;
    if (index_cap && (!d_workspace || workspace_bytes < halo_kcp_ingest_workspace(index_cap, cfg->seg_cap))) return HALO_E_INVAL;
    const kcp::DeviceOps* ops = kcp::device_ops ? kcp::device_ops() : nullptr;
    return ops ? ops->run(cfg, d_stream, d_deliver_summary, d_index, index_cap, d_dgrams, d_segs, d_summary, d_workspace, stream)
               : HALO_E_NODEV;
}

extern "C" HALO_API int halo_kcp_ingest_host(const halo_kcp_config_t* cfg, const uint8_t* stream,
                                             const halo_deliver_summary_t* deliver_summary,
                                             const halo_deliver_index_t* index, uint32_t index_cap,
                                             halo_kcp_dgram_t* dgrams, halo_kcp_seg_t* segs, halo_kcp_summary_t* summary) {
    int rc;
    if ((rc = check(cfg, stream, deliver_summary, index, index_cap, dgrams, segs, summary))) return rc;
    const int32_t mode = cfg->byte_check_mode;
    halo_kcp_summary_t s;  // no alignment asked of host memory: built here, copied out
    memset(&s, 0, sizeof s);
    const uint32_t records = load_u32(deliver_summary);  // halo_deliver_summary_t.records
    const uint32_t nrec = records < index_cap ? records : index_cap;
    bool cut = false;  // a datagram did not fit
    for (uint32_t k = 0; k < nrec; ++k) {
        const uint32_t off = load_u32(reinterpret_cast<const uint8_t*>(index) + 8ull * k + 4);
        if (off == kNotWritten) continue;
        const uint8_t* rec = stream + off;
        const uint32_t w1 = load_u32(rec + 4);
        if (!selected(w1, load_u32(rec + 12), cfg->port)) continue;
        const HostBytes b{rec + deliver::kHdrBytes};
        const uint32_t L = w1 >> 16;
        // the datagram's shape first (its descriptors are written only when all of them fit)
        Dgram d = classify(b, L, mode, [](uint32_t, const Hdr&, uint32_t) {});
        if (d.what == 1u) ++s.ignored;
        if (d.what != 2u) continue;
        if (!cut && s.dgrams < cfg->dgram_cap && (uint64_t)s.segs + d.n_walked <= cfg->seg_cap) {
            const uint32_t j = s.dgrams, first = s.segs;
            uint32_t n_segs = d.n_walked;
            uint64_t hashed = 0;
            if (d.kind == HALO_KCP_DGRAM_KCP) {
                walk(b, L, overhead(mode), d.conv0_lo, d.conv0_hi, [&](uint32_t i, const Hdr& h, uint32_t pos) {
                    uint32_t chk = check_without_hash(mode, h);
                    if (hashes(mode) && cmd_of(h) == kCmdPush) {
                        chk = byte_check_hash(mode, b.p + pos, h.length) == h.hash ? HALO_KCP_SEG_CHECK_PASSED
                                                                                    : HALO_KCP_SEG_CHECK_FAILED;
                        hashed += h.length;
                    }
                    if (chk == HALO_KCP_SEG_CHECK_FAILED && i < n_segs) n_segs = i;  // the first failed check
                    uint32_t w[8];
                    seg_words(h, j, off + deliver::kHdrBytes + pos, chk, w);
                    memcpy(reinterpret_cast<uint8_t*>(segs) + 32ull * (first + i), w, 32);
                });
                if (n_segs < d.n_walked) d.ret = -4;
                ++s.ret_counts[-d.ret];
                ++s.in_pkts;
                s.in_bytes += L;
                if (d.ret) ++s.in_errs;
                else s.in_segs += n_segs;
                s.bytes_hashed += hashed;
            } else {
                ++s.enet_counts[d.conn_type];
            }
            uint32_t w[10];
            dgram_words(d, k, n_segs, first, w);
            memcpy(reinterpret_cast<uint8_t*>(dgrams) + 40ull * j, w, 40);
            ++s.dgrams_written;
            s.segs_written += d.n_walked;
        } else {
            cut = true;
        }
        ++s.dgrams;
        s.segs += d.n_walked;
    }
    memcpy(summary, &s, sizeof s);
    return HALO_OK;
}
