// tx_kcp_host.cc — KCP emit's C entry points (include/halo_rx.h, "KCP emit"): the argument checks
// of halo_kcp_emit_device, answered before any device is looked for, and halo_kcp_emit_host, the
// sequential loop with the same outputs. No HIP: the kernels live in tx_kcp.hip behind
// kcp_emit::device_ops(), and this file compiles alone with g++ (tools/fuzz_kcp_emit.cc drives it
// under ASan/UBSan). The byte check is kcp_check_host.h's, shared with KCP ingest.
#include <string.h>

#include "kcp_check_host.h"
#include "tx_kcp.h"

namespace halo {
namespace kcp_emit {
namespace {

// What both entry points ask
int check(const halo_kcp_emit_config_t* cfg, const void* sessions, uint32_t n_sessions, const void* segs, uint32_t n_segs,
          const void* payload, uint64_t payload_bytes, const void* stream, const void* dgrams, const void* descs,
          const void* status, const void* summary) {
    if (!cfg || !summary) return HALO_E_INVAL;
    if (!kcp::mode_ok(cfg->byte_check_mode) || cfg->src_port > 0xFFFFu) return HALO_E_INVAL;
    if (n_sessions > HALO_KCP_EMIT_MAX || n_segs > HALO_KCP_EMIT_MAX) return HALO_E_INVAL;
    if (n_sessions && (!sessions || !status)) return HALO_E_INVAL;
    if ((n_segs && !segs) || (payload_bytes && !payload)) return HALO_E_INVAL;
    if ((cfg->dgram_cap && (!dgrams || !descs)) || (cfg->stream_cap && !stream)) return HALO_E_INVAL;
    return HALO_OK;
}

Sess load_sess(const halo_kcp_out_session_t* sessions, uint32_t s) {  // no alignment asked of host memory
    Sess x;
    static_assert(sizeof x == sizeof(halo_kcp_out_session_t), "Sess is the record's dwords");
    memcpy(&x, reinterpret_cast<const uint8_t*>(sessions) + 40ull * s, sizeof x);
    return x;
}

}  // namespace
}  // namespace kcp_emit
}  // namespace halo

using namespace halo;  // host_layout.h
using namespace halo::kcp_emit;

extern "C" HALO_API uint64_t halo_kcp_emit_workspace(uint32_t n_sessions, uint32_t n_segs) {
    return kcp_emit::workspace_bytes(n_sessions, n_segs);
}

extern "C" HALO_API int halo_kcp_emit_device(const halo_kcp_emit_config_t* cfg, const halo_kcp_out_session_t* d_sessions,
                                             uint32_t n_sessions, const halo_kcp_seg_t* d_segs, uint32_t n_segs,
                                             const uint8_t* d_payload, uint64_t payload_bytes, uint8_t* d_stream,
                                             halo_kcp_out_dgram_t* d_dgrams, halo_tx_build_desc_t* d_descs, uint8_t* d_status,
                                             halo_kcp_emit_summary_t* d_summary, void* d_workspace, uint64_t workspace_bytes,
                                             halo_stream_t stream) {
    int rc;
    if ((rc = check(cfg, d_sessions, n_sessions, d_segs, n_segs, d_payload, payload_bytes, d_stream, d_dgrams, d_descs, d_status,
                    d_summary)))
        return rc;
    if (misaligned(d_segs, 16) || misaligned(d_dgrams, 16) || misaligned(d_sessions, 8) || misaligned(d_descs, 8) ||
        misaligned(d_summary, 8) || misaligned(d_workspace, 8) || misaligned(d_payload, 4) || misaligned(d_stream, 4))
        return HALO_E_INVAL;
    if (n_sessions && (!d_workspace || workspace_bytes < halo_kcp_emit_workspace(n_sessions, n_segs))) return HALO_E_INVAL;
    const kcp_emit::DeviceOps* ops = kcp_emit::device_ops ? kcp_emit::device_ops() : nullptr;
    return ops ? ops->run(cfg, d_sessions, n_sessions, d_segs, n_segs, d_payload, payload_bytes, d_stream, d_dgrams, d_descs,
                          d_status, d_summary, d_workspace, stream)
               : HALO_E_NODEV;
}

extern "C" HALO_API int halo_kcp_emit_host(const halo_kcp_emit_config_t* cfg, const halo_kcp_out_session_t* sessions,
                                           uint32_t n_sessions, const halo_kcp_seg_t* segs, uint32_t n_segs,
                                           const uint8_t* payload, uint64_t payload_bytes, uint8_t* stream,
                                           halo_kcp_out_dgram_t* dgrams, halo_tx_build_desc_t* descs, uint8_t* status,
                                           halo_kcp_emit_summary_t* summary) {
    int rc;
    if ((rc = check(cfg, sessions, n_sessions, segs, n_segs, payload, payload_bytes, stream, dgrams, descs, status, summary)))
        return rc;
    const int32_t mode = cfg->byte_check_mode;
    const uint32_t H = kcp::overhead(mode);
    halo_kcp_emit_summary_t sum;  // built here, copied out
    memset(&sum, 0, sizeof sum);
    const uint8_t* seg_bytes = reinterpret_cast<const uint8_t*>(segs);
    uint32_t dg_base = 0, dw_base = 0, seg_base = 0;  // of the OK entries so far, as the device's scan sums them
    uint64_t prev_end = 0;
    for (uint32_t s = 0; s < n_sessions; ++s) {
        const Sess x = load_sess(sessions, s);
        const auto tail = [&](uint32_t i) {
            Tail t;
            memcpy(&t, seg_bytes + 32ull * (x.first_seg + i) + 16, sizeof t);
            return t;
        };
        Shape shape{entry_status(x, prev_end, n_segs, H), 0, 0, 0};
        prev_end = (uint64_t)x.first_seg + x.n_segs;
        if (shape.status == HALO_KCP_EMIT_OK)
            shape = kind_of(x) == HALO_KCP_DGRAM_ENET
                        ? enet_shape()
                        : walk(x, H, payload_bytes, tail, [](uint32_t, uint32_t, uint32_t, uint32_t) {},
                               [](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {});
        status[s] = (uint8_t)shape.status;
        ++sum.status_counts[shape.status];
        if (shape.status != HALO_KCP_EMIT_OK) continue;
        if (fits(shape, dg_base, dw_base, seg_base, cfg->dgram_cap, cfg->stream_cap, n_segs)) {
            const uint32_t base = 4u * dw_base;  // the entry's first stream byte
            const auto put_records = [&](uint32_t j, uint32_t rel, uint32_t size, uint32_t n, uint32_t first_i) {
                uint32_t w[4], d[10];
                dgram_words(base + rel, size, n, s, x.first_seg + first_i, w);
                desc_words(base + rel, size, cfg->src_ip, cfg->src_port, x, d);
                memcpy(reinterpret_cast<uint8_t*>(dgrams) + 16ull * (dg_base + j), w, 16);
                memcpy(reinterpret_cast<uint8_t*>(descs) + 40ull * (dg_base + j), d, 40);
                memset(stream + base + rel + size, 0, (0u - size) & 3u);  // the datagram's padding
                sum.out_bytes += size;
            };
            if (kind_of(x) == HALO_KCP_DGRAM_ENET) {
                uint32_t w[5];
                enet_words(x, w);
                memcpy(stream + base, w, 20);
                put_records(0, 0, kcp::kEnetBytes, 0, 0);
            } else {
                walk(x, H, payload_bytes, tail,
                     [&](uint32_t i, uint32_t len, uint32_t data_off, uint32_t rel) {
                         uint32_t lo[4], hw[9];
                         memcpy(lo, seg_bytes + 32ull * (x.first_seg + i), 16);
                         const Tail t = tail(i);
                         uint32_t hash = 0;
                         if ((lo[1] & 0xFFu) == kcp::kCmdPush && kcp::hashes(mode)) {
                             hash = kcp::byte_check_hash(mode, payload + data_off, len);
                             sum.bytes_hashed += len;
                         }
                         header_words(x.conv_lo, x.conv_hi, lo[1], lo[2], lo[3], t.una, len, hash, hw);
                         memcpy(stream + base + rel, hw, H);
                         if (len) memcpy(stream + base + rel + H, payload + data_off, len);
                     },
                     put_records);
            }
            ++sum.sessions_written;
            sum.dgrams_written += shape.dgrams, sum.segs_written += shape.segs, sum.bytes_written += 4ull * shape.dwords;
        }
        ++sum.sessions;
        dg_base += shape.dgrams, dw_base += shape.dwords, seg_base += shape.segs;
    }
    sum.dgrams = dg_base, sum.segs = seg_base, sum.bytes = 4ull * dw_base;
    sum.out_segs = sum.segs_written, sum.out_pkts = sum.dgrams_written;
    memcpy(summary, &sum, sizeof sum);
    return HALO_OK;
}
